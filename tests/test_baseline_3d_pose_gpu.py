"""GPU: K19, the fused BatchNorm1d + ReLU + dropout (+ residual) kernel (csrc/p2c_bnorm.hip, ops.batch_norm_act), and the
Baseline3DPose(Rot) models on it.

(a) K19 against fp64 nn.BatchNorm1d + ReLU (+ residual) on the CPU, train and eval: z, running statistics and every gradient
within 1e-4; bitwise-equal repeats; N = 1 raises; N C >= 2^31 refused by the host check; (b) the hashed dropout: keep fraction,
masks per site / step, replay after restore, the backward's mask; (c) the reference fixtures on the device; (d) one training
step of LitPoseLiftingFlow with each model against the fp64 CPU twin + oracle pose head (unflattened and flat trainer);
(e) graph capture with dropout 0.5; (f) no framework BatchNorm / ReLU / dropout in the device step."""
import copy
import ctypes
import os
import sys

import pytest
import torch

from oracle import pose_head as O

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL, floor=0.0):
    """max |a - b| <= rtol * max(max |b|, floor)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), floor)
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def _bn_pair(C, seed, beta_shift=0.0):
    """(device fp32 BatchNorm1d, CPU fp64 twin) with random affine parameters and running statistics."""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.5 + beta_shift)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref = copy.deepcopy(bn).double()
    return bn.to(dev()), ref


def _run(bn, y, res, g_z, p=0.0, st=None, site=0, relu=True):
    from pedestrians_video_2_carla_amd import ops
    yd = y.clone().requires_grad_(True)
    rd = None if res is None else res.clone().requires_grad_(True)
    bn.weight.grad = bn.bias.grad = None
    z = ops.batch_norm_act(yd, bn, p, st, site, residual=rd, relu=relu)
    z.backward(g_z)
    return z.detach(), yd.grad, bn.weight.grad.clone(), bn.bias.grad.clone(), None if rd is None else rd.grad


# every N in {2, 3, 33, 1030, 4096, 65536} and every C in {1, 7, 52, 200, 1024} at least once
SHAPES = [(2, 7), (3, 1), (33, 52), (1030, 200), (1030, 1), (4096, 1024), (4096, 7), (65536, 1024)]


@pytest.mark.parametrize('N,C', SHAPES)
@pytest.mark.parametrize('training', [True, False])
def test_k19_matches_fp64_batch_norm(N, C, training):
    d = dev()
    bn, ref = _bn_pair(C, N + C)
    bn.train(training), ref.train(training)
    g = torch.Generator().manual_seed(N * 7 + C)
    # (inputs rounded to fp32 first: the twin sees exactly what the kernel sees)
    y = (torch.randn(N, C, generator=g) * 2 + 1).double()
    res = torch.randn(N, C, generator=g).double() if (N + C) % 2 else None
    g_z = torch.randn(N, C, generator=g).double()
    # where the fp64 pre-activation lies within fp32 rounding of 0 the ReLU gate of an fp32 kernel is a coin toss (N = 65536,
    # C = 1024 has a few such elements): the upstream gradient is zero there, so that either gate gives the same gradients
    mean, var = (y.mean(0), y.var(0, unbiased=False)) if training else (ref.running_mean, ref.running_var)
    pre = (y - mean) * (var + ref.eps).rsqrt() * ref.weight.detach() + ref.bias.detach()
    g_z[pre.abs() < 1e-5 * pre.abs().max()] = 0.0
    yr = y.clone().requires_grad_(True)
    rr = None if res is None else res.clone().requires_grad_(True)
    zr = torch.relu(ref(yr))
    zr = zr if rr is None else zr + rr
    zr.backward(g_z)
    f = lambda t: None if t is None else t.float().to(d)   # noqa: E731
    z, gy, gw, gb, gres = _run(bn, f(y), f(res), f(g_z))
    # dy = gamma rstd (g - mean g - xh mean(g xh)) cancels to ~0 for tiny N (N = 2: exactly): there it is judged against 1 % of
    # the scale of its terms, gamma rstd |g|, instead of its own
    rstd = (y.var(0, unbiased=False) + ref.eps).rsqrt() if training else (ref.running_var + ref.eps).rsqrt()
    floor = 1e-2 * float((ref.weight.detach() * rstd).abs().max()) * float(g_z.abs().max()) if N <= 3 else 0.0
    close(z, zr, 'z'), close(gy, yr.grad, 'dy', floor=floor)
    close(gw, ref.weight.grad, 'dgamma'), close(gb, ref.bias.grad, 'dbeta')
    if res is not None:
        close(gres, rr.grad, 'dresidual')
    close(bn.running_mean, ref.running_mean, 'running_mean'), close(bn.running_var, ref.running_var, 'running_var')
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


@pytest.mark.parametrize('N,C', [(4096, 1024), (1030, 7)])
def test_k19_is_bitwise_reproducible(N, C):
    d = dev()
    g = torch.Generator().manual_seed(3)
    y, g_z = torch.randn(N, C, generator=g).to(d), torch.randn(N, C, generator=g).to(d)
    runs = []
    for _ in range(2):
        bn, _ = _bn_pair(C, 9)
        runs.append(_run(bn, y, y * 0.5, g_z) + (bn.running_mean.clone(), bn.running_var.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_row_in_training_raises_like_batch_norm():
    from pedestrians_video_2_carla_amd import ops
    bn, _ = _bn_pair(8, 1)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        ops.batch_norm_act(torch.randn(1, 8, device=dev()), bn, 0.0, None, 0)
    bn.eval()
    assert ops.batch_norm_act(torch.randn(1, 8, device=dev()), bn, 0.0, None, 0).shape == (1, 8)


def test_2_pow_31_elements_are_refused_without_a_launch():
    from pedestrians_video_2_carla_amd import _lib, ops
    lib = _lib.lib()
    N, C = 1 << 21, 1024                     # N C = 2^31: a shape, nothing allocated
    assert N * C >= ops.BNORM_MAX_ELEMENTS
    assert lib.p2c_bnorm_workspace_floats(N, C) == 0 and lib.p2c_bnorm_workspace_floats(N - 1, C) > 0
    fake = torch.empty(16, device=dev())
    d = _lib.BnormDesc()
    d.N, d.C, d.training, d.relu, d.eps, d.momentum = N, C, 1, 1, 1e-5, 0.1
    for f in ('y', 'gamma', 'beta', 'z', 'mean', 'rstd', 'running_mean', 'running_var', 'g_z', 'g_y', 'g_gamma', 'g_beta'):
        setattr(d, f, fake.data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    assert lib.p2c_bnorm_fwd(ctypes.byref(d), fake.data_ptr(), s) == -2
    assert lib.p2c_bnorm_bwd(ctypes.byref(d), fake.data_ptr(), s) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- dropout
def _masks(bn, y, p, st, site):
    """The keep mask of one forward (beta large: the ReLU is the identity, z == 0 exactly where an element was dropped)."""
    from pedestrians_video_2_carla_amd import ops
    yd = y.clone().requires_grad_(True)
    z = ops.batch_norm_act(yd, bn, p, st, site)
    z.backward(torch.ones_like(z))
    return z.detach() != 0


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_keep_fraction_and_streams(p):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    torch.manual_seed(4)
    st = ops.dropout_state(d)
    bn, _ = _bn_pair(256, 2, beta_shift=50.0)
    y = torch.randn(4096, 256, device=d)
    snap = ops.dropout_states_snapshot()
    m0 = _masks(bn, y, p, st, 0)
    m0b = _masks(bn, y, p, st, 0)                # next step
    ops.dropout_states_restore(snap)
    m0r = _masks(bn, y, p, st, 0)                # replays step 0
    m1r = _masks(bn, y, p, st, 1)                # step 1, another site
    n = m0.numel()
    keep = m0.double().mean().item()
    assert abs(keep - (1 - p)) <= 5 * ((p * (1 - p) / n) ** 0.5), keep
    assert torch.equal(m0, m0r) and not torch.equal(m0, m0b) and not torch.equal(m0b, m1r)
    ops.dropout_states_restore(snap)
    m1 = _masks(bn, y, p, st, 1)                 # step 0, site 1
    assert not torch.equal(m0, m1)


def test_dropout_backward_uses_the_forward_mask():
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    torch.manual_seed(6)
    p, N, C = 0.5, 1030, 52
    st = ops.dropout_state(d)
    bn, ref = _bn_pair(C, 3, beta_shift=50.0)
    g = torch.Generator().manual_seed(8)
    y, g_z = torch.randn(N, C, generator=g, dtype=torch.float64), torch.randn(N, C, generator=g, dtype=torch.float64)
    z, gy, gw, gb, _ = _run(bn, y.float().to(d), None, g_z.float().to(d), p=p, st=st, site=3)
    mask = (z != 0).double().cpu()
    assert 0.4 < mask.mean().item() < 0.6
    yr = y.clone().requires_grad_(True)
    zr = torch.relu(ref(yr)) * mask / (1 - p)
    zr.backward(g_z)
    close(z, zr, 'z'), close(gy, yr.grad, 'dy'), close(gw, ref.weight.grad, 'dgamma'), close(gb, ref.bias.grad, 'dbeta')


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.mark.parametrize('name', ['model_baseline3d_a', 'model_baseline3d_rot_b'])
def test_reference_fixture_on_the_device(name):
    from test_baseline_3d_pose import build_model, check_fixture, load_fixture
    d = dev()
    g = load_fixture(name)
    model = build_model(name, g).to(d).train()
    check_fixture(model, g, RTOL, to=lambda t: t.to(d), grad_rtol=5e-4)      # (gradients: test_flow_gpu's BatchNorm rule)


def test_seeded_initial_parameters_survive_the_move_to_the_device():
    from test_baseline_3d_pose import load_fixture
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.baseline_3d_pose import Baseline3DPoseRot
    g = load_fixture('model_baseline3d_init_c')
    torch.manual_seed(1234)
    model = Baseline3DPoseRot(input_nodes=CARLA_SKELETON, linear_size=64, num_stage=3).to(dev())
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), g['sd__' + k]), k


def _flow(cls_name, B=32, T=16, p_dropout=0.0, **kw):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements import baseline_3d_pose
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    # (seed 8: no clip whose untrained prediction puts the neck almost onto the hips -- the hips-neck re-normalisation of
    # ``absolute_loc`` makes such a batch ill-conditioned; seed 5 gives one for Baseline3DPoseRot, where fp32 on the CPU is
    # already 1 % off fp64)
    seed_everything(8)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    model = getattr(baseline_3d_pose, cls_name)(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, p_dropout=p_dropout, **kw)
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform=dm.transform.name)
    return flow, dm


@pytest.mark.parametrize('cls_name', ['Baseline3DPose', 'Baseline3DPoseRot'])
@pytest.mark.parametrize('flatten', [False, True])
def test_training_step_matches_the_cpu_twin(cls_name, flatten):
    """Defaults (linear_size 1024, num_stage 2), B = 32, T = 16, loc_2d_3d, dropout 0: loss and every parameter gradient of one
    training step vs the fp64 CPU twin + the oracle pose head on its locations. Tolerances: test_flow_gpu's LinearAEResidual
    rule (5e-4 of the larger of a gradient's own scale and 1e-3 of the largest gradient: the biases in front of a BatchNorm have
    an analytically zero gradient), widened to twice what an fp32 CPU twin loses against fp64 where that is more (the
    hips-neck re-normalisation of ``absolute_loc`` amplifies rounding when a clip's predicted neck nearly meets its hips)."""
    from pedestrians_video_2_carla_amd import ops
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(cls_name)
    model = flow.movements_model
    twins = {dt: copy.deepcopy(model).to(dt).train() for dt in (torch.float64, torch.float32)}
    trainer = Trainer(device=d, flatten=flatten).setup(flow, dm)
    batch = dm.generate_batch(d)
    frames, targets, meta = batch
    flow.train()
    with ops.grad_sinks(trainer._grad_sinks):        # (the flat trainer: gradients added straight into the flat buffer)
        flow.on_train_batch_start(batch, 0)
        loss = flow.training_step(batch, 0)['loss']
        loss.backward()
    ref = {}
    for dt, twin in twins.items():
        out = twin(frames.to('cpu', dt))
        loc = out[0] if isinstance(out, tuple) else out
        o = O.pose_head(loc, 'absolute_loc', meta['skel_type'].cpu(), gt2d=targets['projection_2d_transformed'].to('cpu', dt),
                        gt3d=targets['absolute_pose_loc'].to('cpu', dt))
        o['loc_2d_3d'].backward()
        ref[dt] = o['loc_2d_3d'].detach()
    l64, l32 = float(ref[torch.float64]), float(ref[torch.float32])
    close(loss, ref[torch.float64], 'loss', rtol=max(1e-4, 2 * abs(l32 - l64) / abs(l64)))
    cpu64, cpu32 = twins[torch.float64], twins[torch.float32]
    top = max(float(pc.grad.abs().max()) for pc in cpu64.parameters() if pc.grad is not None)
    for (n, pg), pc, pc32 in zip(model.named_parameters(), cpu64.parameters(), cpu32.parameters()):
        if pc.grad is None:
            assert pg.grad is None or float(pg.grad.abs().max()) == 0.0, n
            continue
        scale = max(float(pc.grad.abs().max()), 1e-3 * top)
        ref_err = float((pc32.grad.double() - pc.grad).abs().max()) / scale
        err = float((pg.grad.double().cpu() - pc.grad).abs().max())
        assert err <= max(5e-4, 2 * ref_err) * scale, (n, err, scale, ref_err)
    for (n, b), (_, bc) in zip(model.named_buffers(), cpu64.named_buffers()):
        if n.endswith('num_batches_tracked'):
            assert int(b) == int(bc) == 1, n
        else:
            close(b, bc, n)


@pytest.mark.parametrize('cls_name', ['Baseline3DPose', 'Baseline3DPoseRot'])
def test_graph_capture_with_dropout(cls_name):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(cls_name, B=32, T=16, p_dropout=0.5, linear_size=256)
    trainer = Trainer(device=d, use_graph=True).setup(flow, dm)
    batch = dm.generate_batch(d)
    bn = flow.movements_model.baseline.linear_stages[1].batch_norm2
    losses = [float(trainer.train_step(flow, batch, 0))]
    diff, scale = trainer._replay_check
    assert trainer.use_graph and scale > 0 and diff == 0.0, (diff, scale)
    rm, nbt = bn.running_mean.clone(), int(bn.num_batches_tracked)
    for i in range(1, 50):
        losses.append(float(trainer.train_step(flow, batch, i)))
    torch.cuda.synchronize()
    assert all(l == l and abs(l) < float('inf') for l in losses), losses
    assert sum(losses[-5:]) < sum(losses[:5]), losses
    assert int(bn.num_batches_tracked) == nbt + 49 and not torch.equal(bn.running_mean, rm)


@pytest.mark.parametrize('cls_name', ['Baseline3DPose', 'Baseline3DPoseRot'])
def test_no_framework_batch_norm_relu_or_dropout_in_the_device_step(cls_name, monkeypatch):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(cls_name, B=16, T=8, p_dropout=0.5, linear_size=128)
    trainer = Trainer(device=d).setup(flow, dm)
    batch = dm.generate_batch(d)

    def framework(*a, **k):
        raise AssertionError('a framework BatchNorm / ReLU / dropout ran')
    for owner, name in ((torch.nn.BatchNorm1d, 'forward'), (torch.nn.Dropout, 'forward'), (torch.nn.ReLU, 'forward'),
                        (torch.nn.functional, 'batch_norm'), (torch.nn.functional, 'dropout')):
        monkeypatch.setattr(owner, name, framework)
    loss = trainer.train_step(flow, batch, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
