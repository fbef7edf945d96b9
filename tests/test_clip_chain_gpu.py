"""GPU: the MLP chains of the clip kernel (csrc/p2c_train.hip) and of the fused MLP (csrc/p2c_mlp_dev.h) after their diet --
exact k-step counts (no MFMA on zero padding), single-wave layer runs without a workgroup barrier, the suffix sum over time
on the matrix pipe. None of it changes a summation order, so the fused step stays BITWISE equal to the separate kernels; the
persistent form (a workgroup walks two clips: the weight image is staged in the first one only) and the generic shapes are
checked against fp64."""
import copy
import math
import os
import sys

import pytest
import torch

from oracle import pose_head as O

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_gpu import close, dev, make  # noqa: E402


def _trainer(flow, dm):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return Trainer(device=dev()).setup(flow, dm)


def _one_step(monkeypatch, fused, **kw):
    monkeypatch.setenv('P2C_FUSED_TRAIN', fused)
    flow, dm = make(**kw)
    trainer = _trainer(flow, dm)
    trainer.optimizers[0].zero_grad_in_step = False
    batch = dm.generate_batch(dev())
    loss = trainer._forward_backward(flow, batch, 0)
    torch.cuda.synchronize()
    assert (getattr(flow, '_pair_counts', None) is not None) == (fused == '1')
    return (loss.detach().cpu().clone(), flow.logged['train_loss/loc_2d'].cpu().clone(),
            flow.logged['train_loss/loc_3d'].cpu().clone(), trainer.flat.flat_grad.detach().cpu().clone())


@pytest.mark.parametrize('otype', ['pose_changes', 'relative_rot'])
@pytest.mark.parametrize('T', [5, 16])
def test_fused_gradient_against_the_separate_kernels(monkeypatch, otype, T):
    """B = 256, 30 % missing joints, both 6-D kinds, optimizer kept out (P2C_FUSED_UPDATE=0): one step with and without the fused
    step. T = 16: the three losses and the whole flat gradient are the same BITS. T = 5 (eleven of a clip tile's sixteen sample
    columns are padding: zero rows in the time planes, zero x columns): the losses are the same bits; the weight gradient is
    not, before this file existed either -- the separate kernels cut the 1 280 frames into 80 tiles of 16 consecutive rows,
    the fused step into 256 tiles of one clip, so the same per-frame products are added in another grouping (measured: 7.6e-6
    absolute at a gradient scale of order 1). There the rule of test_throughput_forms_match_the_separate_kernels_at_full_size
    holds: 1e-4 of the gradient's scale."""
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    sep = _one_step(monkeypatch, '0', B=256, T=T, missing=0.3, otype=otype)
    fus = _one_step(monkeypatch, '1', B=256, T=T, missing=0.3, otype=otype)
    assert torch.isfinite(sep[3]).all() and sep[3].abs().max() > 0
    names = ('loss', 'loc_2d', 'loc_3d', 'flat gradient')
    for a, b, what in zip(sep, fus, names):
        print(f'T={T} {otype} {what}: max |diff| {(a - b).abs().max().item():.3e} at scale {a.abs().max().item():.3e}')
    for a, b, what in zip(sep[:3], fus[:3], names):
        assert torch.equal(a, b), f'{what}: max |diff| {(a - b).abs().max().item():.3e}'
    if T == 16:
        assert torch.equal(sep[3], fus[3]), f'flat gradient: max |diff| {(sep[3] - fus[3]).abs().max().item():.3e}'
    else:
        close(fus[3], sep[3], 'flat gradient', rtol=1e-4)


@pytest.fixture
def latency_form():
    """train_clip_kernel (a workgroup per clip, persistent beyond one clip per CU) at every batch size; restored afterwards."""
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    prev = lib.p2c_train_step_set_stream_min_batch(1 << 30)
    yield
    lib.p2c_train_step_set_stream_min_batch(prev)


def test_second_clip_of_a_workgroup_matches_cpu_pipeline(monkeypatch, latency_form):
    """B = 258: workgroups 0 and 1 walk two clips, the second one without the image staging that is tied to the first clip's
    barriers. Loss and every parameter gradient against LinearAE in fp64 + the oracle pose head (the rule of
    test_fused_step_matches_cpu_pipeline: 1e-4, or twice the error of the fp32 CPU pipeline)."""
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
    transform = 'hips_neck_bbox'
    flow, dm = make(B=258, T=16, missing=0.1, transform=BaseTransforms[transform])
    cpu_model = copy.deepcopy(flow.movements_model).double()
    trainer = _trainer(flow, dm)
    trainer.optimizers[0].zero_grad_in_step = False
    batch = dm.generate_batch(dev())
    frames, targets, meta = batch
    loss = trainer._forward_backward(flow, batch, 0)
    torch.cuda.synchronize()
    assert getattr(flow, '_pair_counts', None) is not None
    gt2d = targets['projection_2d_transformed' if transform != 'none' else 'projection_2d']
    o = O.pose_head(cpu_model(frames.double().cpu()), 'pose_changes_6d', meta['skel_type'].cpu(), transform=transform,
                    gt2d=gt2d.double().cpu(), gt3d=targets['absolute_pose_loc'].double().cpu())
    o['loc_2d_3d'].backward()
    close(loss, o['loc_2d_3d'], 'loss')
    close(flow.logged['train_loss/loc_2d'], o['loc_2d'], 'loc_2d')
    close(flow.logged['train_loss/loc_3d'], o['loc_3d'], 'loc_3d')
    cpu32 = copy.deepcopy(cpu_model).float()
    o32 = O.pose_head(cpu32(frames.float().cpu()), 'pose_changes_6d', meta['skel_type'].cpu(), transform=transform,
                      gt2d=gt2d.float().cpu(), gt3d=targets['absolute_pose_loc'].float().cpu())
    o32['loc_2d_3d'].backward()
    for (n, p), q, q32 in zip(flow.movements_model.named_parameters(), cpu_model.parameters(), cpu32.parameters()):
        ref_err = (q32.grad.double() - q.grad).abs().max().item() / (q.grad.abs().max().item() + 1e-30)
        close(p.grad, q.grad, n, rtol=max(1e-4, 2 * ref_err))


# widths of the generic-shape case: forward k-steps ceil((n_in + 1) / 4) = 3, 2, 5, 1, 4, 6, 9 and dgrad k-steps
# ceil(n_out / 4) = 5, 1, 4, 6, 9, 3 (layers 1..6) -- every residue mod 4 on both sides, loops with no whole group of four,
# with one and with two; output tiles 1, 2, 1, 1, 2, 3, 1 and m-tiles 1, 2, 1, 1, 2, 3
GENERIC_DIMS = [10, 6, 17, 1, 15, 23, 33, 12]


def test_generic_mlp_with_every_k_tail_matches_fp64():
    """K8 with run-time shapes through ops.fused_mlp, N = 33 rows (three sample tiles, the last one with a single row; run-time
    shapes round the k loops up to whole groups of four steps, shapes known at compile time run the exact count):
    output and every weight and bias gradient against fp64 at the tolerance of tests/test_mlp_gpu.py (2e-5 of the scale).
    (ops.fused_mlp computes no input gradient: dgrad is seen through the weight gradients of the layers below.)"""
    from pedestrians_video_2_carla_amd import ops
    dims = GENERIC_DIMS
    assert {(i + 1 + 3) // 4 % 4 for i in dims[:-1]} == {0, 1, 2, 3} and {(o + 3) // 4 % 4 for o in dims[2:]} == {0, 1, 2, 3}
    assert ops.mlp_supported(dims)
    d = dev()
    g = torch.Generator().manual_seed(11)
    # positive biases keep the narrow ReLU layers (1 and 6 wide) alive, so that every gradient below them is non-zero
    Ws = [(torch.randn(o, i, generator=g) / math.sqrt(i)).to(d).requires_grad_(True) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(torch.rand(o, generator=g) * 0.5 + 0.25).to(d).requires_grad_(True) for o in dims[1:]]
    x = torch.randn(33, dims[0], generator=g).to(d)
    w = torch.randn(33, dims[-1], generator=g).to(d)
    y = ops.fused_mlp(x, Ws, bs)
    (y * w).sum().backward()
    Wr = [p.detach().double().cpu().requires_grad_(True) for p in Ws]
    br = [p.detach().double().cpu().requires_grad_(True) for p in bs]
    h = x.double().cpu()
    for l, (W, b) in enumerate(zip(Wr, br)):
        h = h @ W.t() + b
        if l < len(Wr) - 1:
            h = torch.relu(h)
    (h * w.double().cpu()).sum().backward()
    tol = 2e-5
    err = lambda a, b: (a.detach().double().cpu() - b).abs().max().item() / b.abs().max().item()
    print('forward', f'{err(y, h.detach()):.2e}')
    for l, (p, q) in enumerate(zip(Ws + bs, Wr + br)):
        assert q.grad.abs().max().item() > 0, f'parameter {l}: the reference gradient is zero, the case checks nothing'
        print('parameter', l, f'{err(p.grad, q.grad):.2e}')
    close(y, h, 'forward', rtol=tol)
    for l, (p, q) in enumerate(zip(Ws + bs, Wr + br)):
        close(p.grad, q.grad, f'gradient of parameter {l}', rtol=tol)
