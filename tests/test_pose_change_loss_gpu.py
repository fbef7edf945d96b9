"""GPU: K27 (csrc/p2c_pose_change_loss.hip, ``ops.pose_change_loss``) against the fp64 tensor path on the CPU -- ``_accumulate`` +
``mse_loss`` for the cumulative form, the plain difference for the direct one, ``oracle.pose_head.rotation_6d_to_matrix`` for 6-D
input. Loss within 1e-5 relative (the rtol tests/test_losses_extra.py applies to this loss on the device), gradient within
1e-4 of the largest reference gradient (the parity budget of csrc/p2c_pose_head_dev.h)."""
import ctypes
import functools
import math

import pytest
import torch

from oracle.pose_head import rotation_6d_to_matrix
from pedestrians_video_2_carla_amd.loss.cum_pose_changes import _accumulate

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4
# (B, T, J, max_blocks): one lane; one short chain per joint; the golden shape (78 chains: the second wavefront is partial); the
# other skeletons' joint counts with odd T; B J = 64 and 65 (the wavefront boundary); one workgroup striding over 1040 chains
SHAPES = [(1, 1, 1, 0), (1, 2, 26, 0), (3, 16, 26, 0), (2, 5, 25, 0), (5, 17, 24, 0), (2, 3, 32, 0), (5, 3, 13, 0), (40, 3, 26, 1)]


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def ref_loss(pred64, tgt64, cumulative, reduction):
    """The tensor path in fp64: pred64 (B,T,J,6) or (B,T,J,3,3)."""
    m = rotation_6d_to_matrix(pred64) if pred64.shape[-1] == 6 else pred64
    if cumulative:
        m, tgt64 = _accumulate(m), _accumulate(tgt64)
    return torch.nn.functional.mse_loss(m, tgt64, reduction=reduction)


@functools.lru_cache(maxsize=None)
def problem(B, T, J, six_d, seed=0, noise=0.0):
    """fp32 inputs on the host (shared, never modified): near-rotations, or raw 6-D vectors."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * T + J)
    tgt = rotation_6d_to_matrix(torch.randn(B, T, J, 6, generator=g))
    if six_d:
        pred = torch.randn(B, T, J, 6, generator=g)
    else:
        pred = rotation_6d_to_matrix(torch.randn(B, T, J, 6, generator=g)) + 0.05 * torch.randn(B, T, J, 3, 3, generator=g)
    return pred.contiguous(), tgt.contiguous()


@functools.lru_cache(maxsize=None)
def reference(B, T, J, six_d, cumulative, reduction):
    pred, tgt = problem(B, T, J, six_d)
    p = pred.double().requires_grad_(True)
    loss = ref_loss(p, tgt.double(), cumulative, reduction)
    loss.backward()
    return loss.detach(), p.grad


def check(got_loss, got_grad, want_loss, want_grad, what):
    gl, wl = float(got_loss.detach()), float(want_loss)
    rel = abs(gl - wl) / max(abs(wl), 1e-300)
    scale = want_grad.abs().max().item()
    err = (got_grad.double().cpu() - want_grad).abs().max().item()
    print(f'{what}: loss {gl:.9g} vs {wl:.9g} (rel {rel:.2e}); gradient err {err:.3e} of scale {scale:.3e} ({err / max(scale, 1e-300):.2e})')
    assert math.isfinite(gl) and rel <= LOSS_RTOL, what
    assert math.isfinite(err) and err <= GRAD_RTOL * scale, what


@pytest.mark.parametrize('B,T,J,max_blocks', SHAPES)
def test_loss_and_gradient_match_the_fp64_tensor_path(B, T, J, max_blocks):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    for six_d in (True, False):
        pred, tgt = problem(B, T, J, six_d)
        tgt_d = tgt.to(d)
        for cumulative in (True, False):
            for reduction in ('mean', 'sum'):
                want_loss, want_grad = reference(B, T, J, six_d, cumulative, reduction)
                for g in (1.0, 0.37):
                    p = pred.to(d).requires_grad_(True)
                    loss = ops.pose_change_loss(p, tgt_d, cumulative, reduction, max_blocks=max_blocks)
                    assert loss.shape == () and loss.dtype == torch.float32
                    (loss * g).backward()
                    check(loss, p.grad, want_loss, want_grad * g,
                          f'B{B} T{T} J{J} six_d={six_d} cumulative={cumulative} {reduction} g={g}')


def test_matrices_that_are_not_orthonormal():
    """dM_t = C_{t-1}^T A_t needs the running product itself: a transpose taken for an inverse shows here."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(11)
    for (B, T, J) in ((2, 5, 26), (3, 4, 7), (1, 2, 1)):
        pred, tgt = 0.7 * torch.randn(B, T, J, 3, 3, generator=g), 0.7 * torch.randn(B, T, J, 3, 3, generator=g)
        p64 = pred.double().requires_grad_(True)
        want = ref_loss(p64, tgt.double(), True, 'mean')
        want.backward()
        p = pred.to(d).requires_grad_(True)
        loss = ops.pose_change_loss(p, tgt.to(d), True, 'mean')
        loss.backward()
        check(loss, p.grad, want.detach(), p64.grad, f'not orthonormal B{B} T{T} J{J}')


def test_time_slices_and_view_gradients():
    """The flow hands over ``[:, eval_slice]`` views; a scalar gradient can arrive as a stride-0 or an offset view."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(5)
    big6, bigm = torch.randn(3, 6, 26, 6, generator=g), rotation_6d_to_matrix(torch.randn(3, 6, 26, 6, generator=g))
    tgt = rotation_6d_to_matrix(torch.randn(3, 6, 26, 6, generator=g))
    for big in (big6, bigm):
        b64 = big.double().requires_grad_(True)
        want = ref_loss(b64[:, 1:4], tgt.double()[:, 1:4], True, 'mean')
        (want * 0.37).backward()
        grads = (torch.full((1,), 0.37, device=d).expand(5)[3], torch.full((5,), 0.37, device=d)[1:2].view(()))
        for gview in grads:
            leaf = big.to(d).requires_grad_(True)
            view, tview = leaf[:, 1:4], tgt.to(d)[:, 1:4]
            assert not view.is_contiguous() and not tview.is_contiguous()
            loss = ops.pose_change_loss(view, tview, True, 'mean')
            torch.autograd.backward(loss, gview)
            check(loss, leaf.grad, want.detach(), b64.grad, f'slice of {tuple(big.shape)}')
            assert not leaf.grad[:, 0].any() and not leaf.grad[:, 4:].any()


def test_a_nan_reaches_the_loss_and_runs_are_bit_identical():
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    for six_d in (True, False):
        pred, tgt = problem(5, 17, 24, six_d)
        for cumulative in (True, False):
            runs = []
            for _ in range(2):
                p = pred.to(d).requires_grad_(True)
                loss = ops.pose_change_loss(p, tgt.to(d), cumulative, 'mean')
                loss.backward()
                runs.append((loss.detach().clone(), p.grad.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            bad = pred.clone()
            bad[3, 9, 11].view(-1)[1] = float('nan')
            assert torch.isnan(ops.pose_change_loss(bad.to(d), tgt.to(d), cumulative, 'mean'))
            bad_t = tgt.clone()
            bad_t[4, 16, 23, 2, 2] = float('nan')
            assert torch.isnan(ops.pose_change_loss(pred.to(d), bad_t.to(d), cumulative, 'sum'))


def test_refusals_launch_nothing_and_an_empty_batch_is_no_work():
    """Sentinels in every buffer a launch would write stay as they are."""
    from pedestrians_video_2_carla_amd import _lib
    lib, d = _lib.lib(), dev()
    B, T, J = 2, 3, 4
    pred, tgt = torch.randn(B, T, J, 3, 3, device=d), torch.randn(B, T, J, 3, 3, device=d)
    gl = torch.ones(1, device=d)

    def fresh():
        probe = _lib.PoseChangeLossDesc()
        probe.B, probe.T, probe.J, probe.cumulative, probe.mean = B, T, J, 1, 1
        n = lib.p2c_pose_change_loss_workspace_floats(ctypes.byref(probe))
        assert n > 0
        return torch.full((n,), -7.0, device=d), torch.full((1,), -7.0, device=d), torch.full_like(pred, -7.0)

    def call(fn, ws_t, loss_t, gp_t, **over):
        desc = _lib.PoseChangeLossDesc()
        vals = dict(B=B, T=T, J=J, pred_is_6d=0, cumulative=1, mean=1, max_blocks=0, pred=pred.data_ptr(), target=tgt.data_ptr(),
                    workspace=ws_t.data_ptr(), loss=loss_t.data_ptr(), grad_loss=gl.data_ptr(), grad_pred=gp_t.data_ptr())
        vals.update(over)
        for k, v in vals.items():
            setattr(desc, k, v)
        with torch.cuda.device(d):
            return fn(ctypes.byref(desc), torch.cuda.current_stream().cuda_stream)

    refused = [(dict(pred=None), -1), (dict(target=None), -1), (dict(workspace=None), -1), (dict(T=0), -2), (dict(J=0), -2),
               (dict(B=-1), -2), (dict(max_blocks=-1), -2), (dict(pred_is_6d=2), -3), (dict(cumulative=-1), -3), (dict(mean=2), -3),
               (dict(B=238609295, T=1, J=1), -2), (dict(B=9177281, T=1, J=26), -2)]       # 2^31 limit: sizes only, the small buffers
    for fn, extra in ((lib.p2c_pose_change_loss_fwd, [(dict(loss=None), -1)]),
                      (lib.p2c_pose_change_loss_bwd, [(dict(grad_pred=None), -1), (dict(grad_loss=None), -1)])):
        ws, loss, gp = fresh()
        for over, rc in refused + extra:
            assert call(fn, ws, loss, gp, **over) == rc, (fn, over)
        assert call(fn, ws, loss, gp, B=0) == 0                                     # an empty batch: nothing to do
        torch.cuda.synchronize()
        assert bool((ws == -7).all()) and float(loss) == -7 and bool((gp == -7).all())
    # and the same descriptor without an override does launch
    ws, loss, gp = fresh()
    assert call(lib.p2c_pose_change_loss_fwd, ws, loss, gp) == 0 and call(lib.p2c_pose_change_loss_bwd, ws, loss, gp) == 0
    torch.cuda.synchronize()
    want = torch.nn.functional.mse_loss(_accumulate(pred.double().cpu()), _accumulate(tgt.double().cpu()))
    assert abs(float(loss) - float(want)) <= LOSS_RTOL * float(want) and not bool((gp == -7).any())


def test_the_loss_functions_take_the_kernel_on_device_tensors(monkeypatch):
    from pedestrians_video_2_carla_amd import ops
    from pedestrians_video_2_carla_amd.loss import LossModes
    d = dev()
    pred, tgt = problem(3, 16, 26, True)
    calls = []
    real = ops.pose_change_loss
    monkeypatch.setattr(ops, 'pose_change_loss', lambda *a, **k: calls.append(k.get('cumulative')) or real(*a, **k))
    for mode, cumulative in (('pose_changes', False), ('cum_pose_changes', True)):
        fn, crit = LossModes[mode].value
        got = fn(criterion=crit, pose_inputs=pred.to(d), targets={'pose_changes': tgt.to(d)})
        want, _ = reference(3, 16, 26, True, cumulative, crit.reduction)
        assert calls[-1] is cumulative and abs(float(got) - float(want)) <= LOSS_RTOL * float(want)
    n = len(calls)
    monkeypatch.setenv('P2C_PCL_FRAMEWORK', '1')                                    # the comparison arm: tensor ops on the device
    fn, crit = LossModes.cum_pose_changes.value
    got = fn(criterion=crit, pose_inputs=pred.to(d), targets={'pose_changes': tgt.to(d)})
    assert len(calls) == n and got.is_cuda
    assert abs(float(got) - float(reference(3, 16, 26, True, True, 'mean')[0])) <= 1e-4 * float(got)
    monkeypatch.delenv('P2C_PCL_FRAMEWORK')
    assert fn(criterion=torch.nn.L1Loss(), pose_inputs=pred.to(d), targets={'pose_changes': tgt.to(d)}).is_cuda and len(calls) == n
