"""K37 (csrc/p2c_resample.hip) on the device: against the fp64 definition in matrix space, the samples that must be copies, bit
stability across grids, requests, views and cuts of the video, NaN clips, the dispatch and the C ABI's refusals, and
``Trainer.predict_carla`` with a rate.

The allowance is the project's rule (tests/test_carla_pose_gpu.py): what the fp32 tensor restatement of the definition, run on
the device (``P2C_RESAMPLE_FRAMEWORK=1``), is from fp64 on the same inputs is measured, and the kernel gets four times that, with
the floor ``MATRIX_FLOOR``. Rows are compared as the matrices ``carla_pose_import`` makes of them in fp64: Euler rows are ill
conditioned near +-90 degrees of pitch, which the inputs include.
"""
import functools
import math

import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import resample as rs
from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
from test_carla_pose_gpu import MATRIX_FLOOR

pytestmark = pytest.mark.gpu

# (N, T, J, max_blocks): the smallest case that interpolates at all; under one wavefront; a partial last wavefront; several
# workgroups, the root rows starting inside one; another J; two workgroups striding
SHAPES = [(1, 2, 1, 0), (1, 2, 26, 0), (3, 5, 26, 0), (2, 40, 26, 0), (2, 7, 5, 0), (2, 40, 26, 2)]
RATES = [(30, 25), (25, 30), (30, 120), (30, 10), (30, 30)]
LOC_FLOOR = 1e-6


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def problem(N, T, J, seed=0):
    """fp32 rows on the host: locations of unit scale, yaw and roll over +-180 degrees, pitch over +-89."""
    g = torch.Generator().manual_seed(1000 * N + 10 * T + J + seed)

    def make(*lead):
        loc = torch.randn(*lead, 3, generator=g)
        u = torch.rand(*lead, 3, generator=g) * 2 - 1
        return torch.cat((loc, u * torch.tensor([89.0, 180.0, 180.0])), -1)
    return make(N, T, J), make(N, T)


@functools.lru_cache(maxsize=None)
def reference(N, T, J, src, dst, mode='slerp'):
    """The fp64 definition on the host, on the fp32 inputs of ``problem``: rows, their matrices, and (i0, frac)."""
    bones, root = problem(N, T, J)
    b, r = ops.resample_carla_rows(bones.double(), root.double(), src_fps=src, dst_fps=dst, mode=mode)
    i0, frac = rs.sample_positions(0, b.shape[1], rs.rate_ratio(src, dst))
    return b, r, ops.carla_pose_import(b)[1], ops.carla_pose_import(r.unsqueeze(-2))[1], i0, frac


def errors(rows, want_rows, want_rot):
    """(largest matrix entry difference, largest location difference) of device rows against the fp64 reference."""
    rows = rows.double().cpu()
    assert rows.shape == want_rows.shape
    rot = ops.carla_pose_import(rows if rows.ndim == 4 else rows.unsqueeze(-2))[1]
    return float((rot - want_rot).abs().max()), float((rows[..., :3] - want_rows[..., :3]).abs().max())


def kernel(bones, root, src, dst, **kw):
    out = ops.resample_carla_rows(bones, root, src_fps=src, dst_fps=dst, **kw)
    torch.cuda.synchronize()
    return out


def framework(monkeypatch, bones, root, src, dst, **kw):
    with monkeypatch.context() as m:
        m.setenv('P2C_RESAMPLE_FRAMEWORK', '1')
        m.setattr(_lib, 'lib', no_library)
        return kernel(bones, root, src, dst, **kw)


def no_library():
    raise AssertionError('the library was asked for: a launch where none belongs')


@pytest.mark.parametrize('src,dst', RATES)
@pytest.mark.parametrize('N,T,J,max_blocks', SHAPES)
def test_against_fp64_and_bit_stability(N, T, J, max_blocks, src, dst, monkeypatch):
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    want_b, want_r, want_b_rot, want_r_rot, i0, frac = reference(N, T, J, src, dst)
    K = rs.output_count(T - 1, src / dst)
    got_b, got_r = kernel(bones, root, src, dst, max_blocks=max_blocks)
    assert got_b.shape == (N, K, J, 6) and got_r.shape == (N, K, 6) and got_b.dtype == torch.float32 and got_b.is_cuda
    fw_b, fw_r = framework(monkeypatch, bones, root, src, dst)
    scale = max(float(bones[..., :3].abs().max()), float(root[..., :3].abs().max()))
    for what, got, fw, want, want_rot in (('bones', got_b, fw_b, want_b, want_b_rot), ('root', got_r, fw_r, want_r, want_r_rot)):
        fw_rot_err, fw_loc_err = errors(fw, want, want_rot)
        rot_err, loc_err = errors(got, want, want_rot)
        rot_tol, loc_tol = max(4 * fw_rot_err, MATRIX_FLOOR), max(4 * fw_loc_err, LOC_FLOOR * scale)
        print(f'({N},{T},{J}) cap {max_blocks} {src}->{dst} {what}: tensor restatement {fw_rot_err:.3e} / {fw_loc_err:.3e}, '
              f'K37 {rot_err:.3e} / {loc_err:.3e} from fp64 (matrix entries / locations; allowed {rot_tol:.3e} / {loc_tol:.3e})')
        assert math.isfinite(rot_err) and rot_err <= rot_tol, what
        assert math.isfinite(loc_err) and loc_err <= loc_tol, what
    # exact samples: frac == 0 is a copy of the source row
    exact = (frac == 0).to(dev())
    idx = i0.to(dev())[exact]
    assert torch.equal(got_b[:, exact], bones[:, idx]) and torch.equal(got_r[:, exact], root[:, idx])
    if (src, dst) == (30, 30):
        assert torch.equal(got_b, bones) and torch.equal(got_r, root)
    if (src, dst) == (30, 10):
        assert torch.equal(got_b, bones[:, ::3]) and torch.equal(got_r, root[:, ::3])
    # bit stability: a repeat, the full grid, without the root rows, from a strided view
    again_b, again_r = kernel(bones, root, src, dst, max_blocks=max_blocks)
    assert torch.equal(again_b, got_b) and torch.equal(again_r, got_r)
    if max_blocks:
        full_b, full_r = kernel(bones, root, src, dst)
        assert torch.equal(full_b, got_b) and torch.equal(full_r, got_r)
    alone_b, none = kernel(bones, None, src, dst, max_blocks=max_blocks)
    assert none is None and torch.equal(alone_b, got_b)
    wide_b, wide_r = torch.zeros(N, T, J, 8, device=dev()), torch.zeros(N, 2 * T, 6, device=dev())
    wide_b[..., 1:7], wide_r[:, ::2] = bones, root
    view_b, view_r = kernel(wide_b[..., 1:7], wide_r[:, ::2], src, dst, max_blocks=max_blocks)
    assert torch.equal(view_b, got_b) and torch.equal(view_r, got_r)


@pytest.mark.parametrize('src,dst', [(30, 25), (25, 30)])
def test_pushed_chunks_carry_the_bits_of_the_uncut_video(src, dst, monkeypatch):
    chunks = (1, 3, 1, 7, 2, 9, 17)
    N, T, J = 2, sum(chunks), 26
    assert T == 40
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    stream = CarlaResampler(src, dst)
    whole_b, whole_r = stream.resample(bones, root)
    pieces, t = [], 0
    for n in chunks:
        pieces.append(stream.push(bones[:, t:t + n], root[:, t:t + n]))
        t += n
    torch.cuda.synchronize()
    got_b, got_r = torch.cat([p[0] for p in pieces], 1), torch.cat([p[1] for p in pieces], 1)
    assert got_b.shape == whole_b.shape and torch.equal(got_b, whole_b) and torch.equal(got_r, whole_r)
    assert stream.frames == T and stream.outputs == whole_b.shape[1]
    # a push that yields nothing: empty tensors, no launch
    slow = CarlaResampler(30, 10)
    first = slow.push(bones[:, :1], root[:, :1])
    assert torch.equal(first[0], bones[:, :1]) and torch.equal(first[1], root[:, :1])
    with monkeypatch.context() as m:
        m.setattr(_lib, 'lib', no_library)
        b, r = slow.push(bones[:, 1:3], root[:, 1:3])
    assert b.shape == (N, 0, J, 6) and r.shape == (N, 0, 6) and b.is_cuda and b.dtype == torch.float32
    b, r = slow.push(bones[:, 3:5], root[:, 3:5])
    assert torch.equal(b, bones[:, 3:4]) and torch.equal(r, root[:, 3:4])
    with pytest.raises((ValueError, RuntimeError)):
        slow.push(bones[:1, 5:6], root[:1, 5:6])


@pytest.mark.parametrize('src,dst', [(30, 25), (25, 30)])
def test_hold_is_the_gather(src, dst):
    N, T, J = 2, 40, 26
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    b, r = kernel(bones, root, src, dst, mode='hold')
    idx = [math.floor(k * (src / dst)) for k in range(b.shape[1])]
    assert b.shape[1] == rs.output_count(T - 1, src / dst)
    assert torch.equal(b, bones[:, idx]) and torch.equal(r, root[:, idx])
    assert torch.equal(kernel(bones, root, src, dst, mode='hold', max_blocks=2)[0], b)


def test_a_nan_clip_stays_nan_and_touches_nothing_else():
    N, T, J = 3, 9, 26
    bones, root = (t.to(dev()).clone() for t in problem(N, T, J))
    bones[1], root[1] = float('nan'), float('nan')
    for mode in ('slerp', 'hold'):
        b, r = kernel(bones, root, 30, 25, mode=mode)
        assert bool(torch.isnan(b[1]).all()) and bool(torch.isnan(r[1]).all())
        for n in (0, 2):
            alone_b, alone_r = kernel(bones[n:n + 1], root[n:n + 1], 30, 25, mode=mode)
            assert torch.equal(b[n:n + 1], alone_b) and torch.equal(r[n:n + 1], alone_r)
            assert not bool(torch.isnan(b[n]).any()) and not bool(torch.isnan(r[n]).any())


def test_dispatch(monkeypatch):
    N, T, J, src, dst = 3, 5, 26, 30, 25
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    want_b, want_r, want_b_rot, want_r_rot, _, _ = reference(N, T, J, src, dst)
    fw_b, fw_r = framework(monkeypatch, bones, root, src, dst)           # the library is not asked for
    assert fw_b.dtype == torch.float32 and fw_b.is_cuda
    fw_err, fw_loc = errors(fw_b, want_b, want_b_rot)
    tol = max(4 * fw_err, MATRIX_FLOOR)
    with monkeypatch.context() as m:
        m.setattr(_lib, 'lib', no_library)
        d_b, d_r = kernel(bones.double(), root.double(), src, dst)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ac_b, _ = kernel(bones, root, src, dst)
    assert d_b.dtype == torch.float64 and d_b.is_cuda and d_r.dtype == torch.float64
    err64, loc64 = errors(d_b, want_b, want_b_rot)
    err_r64, _ = errors(d_r, want_r, want_r_rot)
    print(f'fp64 on the device {err64:.3e} / {loc64:.3e}, fp32 tensor restatement {fw_err:.3e} / {fw_loc:.3e} (allowed {tol:.3e})')
    assert err64 <= tol and err_r64 <= tol and fw_err <= tol
    assert errors(ac_b, want_b, want_b_rot)[0] <= tol
    got_b, _ = kernel(bones, root, src, dst)
    assert errors(got_b, want_b, want_b_rot)[0] <= tol


def test_abi_refusals_come_before_any_launch():
    lib = _lib.lib()
    N, T, J, K = 2, 4, 3, 4
    bones, root = torch.zeros(N, T, J, 6, device=dev()), torch.zeros(N, T, 6, device=dev())
    cb, cr = torch.zeros(N, J, 6, device=dev()), torch.zeros(N, 6, device=dev())
    out_b, out_r = torch.zeros(N, K, J, 6, device=dev()), torch.zeros(N, K, 6, device=dev())
    base = dict(bones=bones.data_ptr(), root=root.data_ptr(), carry_bones=cb.data_ptr(), carry_root=cr.data_ptr(),
                out_bones=out_b.data_ptr(), out_root=out_r.data_ptr(), N=N, T=T, J=J, K=K, first_output=0, first_frame=0, ratio=1.0,
                mode=0, max_blocks=0)

    def call(**changes):
        a = {**base, **changes}
        return lib.p2c_carla_resample_fwd(*a.values(), None)

    for changes in (dict(N=-1), dict(T=-1), dict(K=-1), dict(first_output=-1), dict(first_frame=-1), dict(max_blocks=-1),
                    dict(J=0), dict(N=2 ** 30, K=2 ** 10), dict(ratio=float('nan')), dict(ratio=float('inf')), dict(ratio=0.0),
                    dict(ratio=-1.0), dict(ratio=2.0 ** -11), dict(ratio=2049.0), dict(mode=2), dict(mode=-1)):
        assert call(**changes) == -2, changes
    assert call(N=-1, bones=None) == -2                                          # shapes are looked at first
    for changes in (dict(bones=None), dict(out_bones=None), dict(out_root=None), dict(root=None), dict(carry_bones=None),
                    dict(carry_root=None)):
        assert call(**changes) == -1, changes
    assert call(N=0) == 0 and call(K=0) == 0
    torch.cuda.synchronize()
    assert float(out_b.abs().sum()) == 0.0 and float(out_r.abs().sum()) == 0.0   # nothing ran
    bones.fill_(1.0), root.fill_(2.0)
    assert call() == 0 and call(root=None, out_root=None, carry_root=None) == 0 and call(carry_bones=None, carry_root=None) == 0
    torch.cuda.synchronize()
    assert float(out_b.min()) == 1.0 and float(out_r.min()) == 2.0
    # an index outside the frames is clamped, never followed: outputs 0..3 at ratio 2 sit at frames 0, 2, 4, 6 of 4
    bones[:, 3] = 5.0
    assert call(ratio=2.0) == 0
    torch.cuda.synchronize()
    assert [float(v) for v in out_b[0, :, 0, 0]] == [1.0, 1.0, 5.0, 5.0]


def test_predict_carla_at_a_rate():
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    seed_everything(11)
    B, T = 2, 8
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
    batches = [dm.generate_batch(dev()), dm.generate_batch(dev())]
    plain = trainer.predict_carla(flow, batches)
    same = trainer.predict_carla(flow, batches, src_fps=None, out_fps=None)
    fast = trainer.predict_carla(flow, batches, src_fps=30, out_fps=20)
    torch.cuda.synchronize()
    stream = CarlaResampler(30, 20)
    for (b, r, meta), (sb, sr, _), (fb, fr, fmeta) in zip(plain, same, fast):
        assert torch.equal(sb, b) and torch.equal(sr, r)
        wb, wr = stream.resample(b, r)
        K = rs.output_count(b.shape[1] - 1, 1.5)
        assert fb.is_cuda and fb.shape == (B, K, 26, 6) and fr.shape == (B, K, 6) and fmeta is meta
        assert torch.equal(fb, wb) and torch.equal(fr, wr)
        assert torch.equal(fb[:, ::2], b[:, ::3])
